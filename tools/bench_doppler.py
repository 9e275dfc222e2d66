#!/usr/bin/env python
"""tools/bench_doppler.py -- time the Doppler moments (kidmp_doppler_moments_device, one launch of kidmp::k_doppler_moments)
on one MI355X beside the two profile diagnostics of the same state that come closest and a torch composite of the same
numbers.

Workloads: 10^5 and 10^4 mixed-phase columns x 120 levels (BASELINE config 3), fp64, after one column step, state in HBM.
All variants run in ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its
own and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  doppler_all    all nine profiles (w given)
  doppler_3      dbz + vd + sw
  doppler_vd     vd alone
  dbz            kidmp_column_outputs_device, dbz alone, on the same state
  fall_all       kidmp_fall_speeds_device, all eleven profiles
  composite      the nine profiles from torch operations on the device tensors (checked against doppler_all once)
Algorithmic bytes per column of a doppler_* variant: (7 state profiles + w read + the requested ones written) * nz * 8;
its share of 8 TB/s is printed.  Prints one line per variant and workload and ONE JSON line at the end; the lines also go
to --out (profiles/r14_doppler.txt) under a header with the date and the library's fingerprint."""
import argparse
import datetime
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ = 120
HBM_PEAK = 8.0e12


def torch_composite(c, dev, w):
    """tests/doppler_ref.py in torch, on device tensors [ncol, nz]: the nine profiles."""
    import torch
    import doppler_ref as r
    import refl_oracle as ro
    G = math.gamma
    t, p = dev["t"], dev["p"]
    qv = torch.clamp(dev["qv"], min=1e-10)
    rho = 0.622 * p / (ro.R * t * (qv + 0.622))
    rhof = torch.sqrt(r.RHO_NOT / rho)
    zero = torch.zeros_like(t)
    tiny = torch.full_like(t, 1.e-22)
    pr, ps, pg = dev["qr"] > ro.R1, dev["qs"] > ro.R2, dev["qg"] > ro.R2
    # rain, M:4997-5004 and M:5130
    rr = torch.where(pr, dev["qr"] * rho, ro.R1)
    nr = torch.where(pr, torch.clamp(dev["nr"] * rho, min=ro.R2), ro.R1)
    lamr = (ro.am_r * c["crg"][2] * c["org2"] * nr / rr) ** (1. / 3.)
    mvd_r = torch.where(pr, 3.672 / lamr, 50.E-6)
    ze_r = torch.where(pr, nr * c["org2"] * lamr * c["crg"][3] / lamr ** 7, tiny)
    vz_r = torch.where(pr, rhof * r.av_r * 7. * lamr ** 7 / (lamr + r.fv_r) ** 8, zero)
    v2_r = torch.where(pr, (rhof * r.av_r) ** 2 * 56. * lamr ** 7 / (lamr + 2. * r.fv_r) ** 9, zero)
    # snow, M:5031-5081 and M:5131-5132
    rs = torch.where(ps, dev["qs"] * rho, ro.R1)
    tc0 = torch.clamp(t - 273.15, max=-0.1)
    fit = lambda a, x: (a[0] + a[1] * tc0 + a[2] * x + a[3] * tc0 * x + a[4] * tc0 * tc0 + a[5] * x * x + a[6] * tc0 * tc0 * x   # noqa: E731
                        + a[7] * tc0 * x * x + a[8] * tc0 * tc0 * tc0 + a[9] * x * x * x)
    smob = rs * c["oams"]
    moment = lambda x: 10.0 ** fit(ro.sa, x) * smob ** fit(ro.sb, x)   # noqa: E731
    ze_s = torch.where(ps, (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI) * (ro.am_s / 900.0) * (ro.am_s / 900.0) * moment(c["cse"][2]), tiny)
    Mrat = smob / moment(c["cse"][0])
    mm = Mrat ** r.mu_s
    A = lambda b, f: (r.Kap0 * G(5. + b) * (Mrat * r.Lam0 + f) ** -(5. + b)   # noqa: E731
                      + r.Kap1 * mm * G(5. + r.mu_s + b) * (Mrat * r.Lam1 + f) ** -(5. + r.mu_s + b))
    a0 = A(0., 0.)
    vz_s = torch.where(ps, rhof * r.av_s * A(r.bv_s, r.fv_s) / a0, zero)
    v2_s = torch.where(ps, (rhof * r.av_s) ** 2 * A(2. * r.bv_s, 2. * r.fv_s) / a0, zero)
    # graupel, M:5086-5103 and M:5133-5135
    rg = torch.where(pg, dev["qg"] * rho, ro.R1)
    slw = (t < 270.65) & pr & (mvd_r > 100.E-6)
    xslw1 = torch.where(slw, 4.01 + torch.log10(mvd_r), 0.01)
    ygra1 = 4.31 + torch.log10(torch.clamp(rg, min=5.E-5))
    zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1))
    n0 = torch.clamp(10. ** zans1, min=ro.gonv_min, max=ro.gonv_max)
    n0 = torch.flip(torch.cummin(torch.flip(n0, [1]), 1).values, [1])
    lam_exp = (n0 * ro.am_g * c["cgg"][0] / rg) ** 0.25
    lamg = lam_exp * (c["cgg"][2] * c["ogg2"] * c["ogg1"]) ** c["obmg"]
    ilamg = 1. / lamg
    ze_g = torch.where(pg, (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI) * (ro.am_g / 900.0) * (ro.am_g / 900.0)
                       * (n0 / (c["cgg"][1] * lam_exp) * lamg) * c["cgg"][3] * ilamg ** 7, tiny)
    vz_g = torch.where(pg, rhof * r.av_g * (G(7. + r.bv_g) / G(7.)) * ilamg ** r.bv_g, zero)
    v2_g = torch.where(pg, (rhof * r.av_g) ** 2 * (G(7. + 2. * r.bv_g) / G(7.)) * ilamg ** (2. * r.bv_g), zero)
    # the moments
    some = pr | ps | pg
    W = torch.where(pr, ze_r, zero) + torch.where(ps, ze_s, zero) + torch.where(pg, ze_g, zero)
    Ws = torch.where(some, W, 1.0)
    V = torch.where(some, (ze_r * vz_r + ze_s * vz_s + ze_g * vz_g) / Ws, zero)
    m2 = torch.where(some, (ze_r * v2_r + ze_s * v2_s + ze_g * v2_g) / Ws, zero)
    dbz_of = lambda ze: 10. * torch.log10(ze * 1.e18)   # noqa: E731
    return dict(dbz=dbz_of(ze_r + ze_s + ze_g), vd=torch.where(some, V - w, zero), sw=torch.sqrt(torch.clamp(m2 - V * V, min=0.)),
                vz_r=vz_r, vz_s=vz_s, vz_g=vz_g, dbz_r=dbz_of(ze_r), dbz_s=dbz_of(ze_s), dbz_g=dbz_of(ze_g))


def measure(a, c, ncol, lines):
    import torch
    import cases
    from kid_amd import DOPPLER_INPUTS, DOPPLER_NAMES, FALL_INPUTS, ThompsonMP

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # the state after one step
    ins = {k: dev[k] for k in DOPPLER_INPUTS}
    fall_ins = {k: dev[k] for k in FALL_INPUTS}
    w = dev["w"]
    variants = {
        "doppler_all": (lambda: m.doppler_moments(ins, w), len(DOPPLER_NAMES)),
        "doppler_3": (lambda: m.doppler_moments(ins, w, want=("dbz", "vd", "sw")), 3),
        "doppler_vd": (lambda: m.doppler_moments(ins, w, want=("vd",)), 1),
        "dbz": (lambda: m.column_outputs(dev, dbz=True, radii=False), None),
        "fall_all": (lambda: m.fall_speeds(fall_ins), None),
        "composite": (lambda: torch_composite(c, ins, w), None),
    }
    got, comp = m.doppler_moments(ins, w), torch_composite(c, ins, w)
    # dB for the reflectivities; relative to the profile's own maximum for the speeds
    diff = {n: float((got[n] - comp[n]).abs().max() / (1.0 if n.startswith("dbz") else got[n].abs().max().clamp(min=1e-300)))
            for n in DOPPLER_NAMES}
    say("ncol=%-6d composite - doppler_all, max |difference| (dbz*: dB; else / max |profile|): %s"
        % (ncol, "  ".join("%s %.1e" % (n, d) for n, d in diff.items())))
    for _ in range(a.warmup):
        for fn, _n in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, (fn, _n) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"ncol": ncol, "nz": NZ, "reps": a.reps, "composite_max_diff": diff}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        nout = variants[k][1]
        extra = ""
        if nout is not None:
            res[k]["algo_bytes_per_column"] = (len(DOPPLER_INPUTS) + 1 + nout) * NZ * 8
            res[k]["share_of_8TBs"] = res[k]["algo_bytes_per_column"] * ncol / (res[k]["ms_median"] * 1e-3) / HBM_PEAK
            extra = "   %6d B/column -> %5.1f %% of 8 TB/s" % (res[k]["algo_bytes_per_column"], 100.0 * res[k]["share_of_8TBs"])
        say("ncol=%-6d %-12s median %8.4f ms   min %8.4f   max %8.4f%s" % (ncol, k, res[k]["ms_median"], min(t), max(t), extra))
    ms = {k: res[k]["ms_median"] for k in variants}
    res["ratios"] = {"doppler_vd/dbz": ms["doppler_vd"] / ms["dbz"], "doppler_3/dbz": ms["doppler_3"] / ms["dbz"],
                     "doppler_all/fall_all": ms["doppler_all"] / ms["fall_all"], "doppler_all/composite": ms["doppler_all"] / ms["composite"],
                     "doppler_all/doppler_vd": ms["doppler_all"] / ms["doppler_vd"]}
    say("ncol=%-6d ratios: %s" % (ncol, "  ".join("%s %.3f" % kv for kv in res["ratios"].items())))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_doppler.txt"))
    a = ap.parse_args()
    import torch
    import doppler_ref as ref
    import kid_amd
    from oracle.oracle import Oracle
    if not torch.cuda.is_available():
        sys.exit("bench_doppler: no GPU visible (this measurement has no CPU path)")
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_doppler.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0)),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = [measure(a, c, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "doppler_moments", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
