#!/usr/bin/env python
"""tools/bench_lidar.py -- time the lidar operator (kidmp_lidar_profiles_device, one launch of kidmp::k_lidar_profiles) on
one MI355X beside the launches of the same state that come closest and a torch composite of the same numbers.

Workloads: 10^5 and 10^4 mixed-phase columns x 120 levels (BASELINE config 3), fp64, after one column step, state in HBM.
All variants run in ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its
own and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  lidar_all      all fourteen profiles and the summary
  lidar_att_up   att_up alone (the scans and the exponentials, one store)
  lidar_ext      ext alone (no scan, no exponential, dz not read)
  spectra_par    kidmp_size_spectra_device, the eleven parameters only: the same load
  summary        kidmp_column_summary_device on the same state
  composite      the fourteen profiles from size_spectra's parameters with torch operations and cumsum (checked against
                 lidar_all once)
Algorithmic bytes per column of a lidar_* variant: (11 state profiles read + the requested ones written) * nz * 8 (+ 64 for
the summary; dz is one shared profile); its share of 8 TB/s is printed, and every time's ratio to spectra_par.  Prints one
line per variant and workload and ONE JSON line at the end; the lines also go to --out (profiles/r22_lidar.txt) under a
header with the date and the library's fingerprint."""
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
NT_C = 100.0e6                                     # the context's droplet number (set_Nc = 100 cm-3)
K_B = 1.380649e-23
CFG = dict(s_ratio=(18.8, 25.0, 18.8, 25.0, 25.0), eta=0.7, c_mol=6.2446e-32, beta_detect=2.0e-5, trans_lost=2.5e-3)


def torch_composite(m, dev, dz):
    """tests/lidar_ref.py in torch, from the parameters size_spectra gives: the fourteen profiles, [ncol, nz]."""
    import torch
    par = m.size_spectra(dev, ("lam_c", "nu_c", "lam_i", "n0_i", "lam_r", "n0_r", "smob", "lam_g", "n0_g"))
    zero = torch.zeros_like(dev["t"])

    def expo(x):
        lam = par["lam_" + x]
        return torch.where(lam > 0, math.pi * par["n0_" + x] / torch.where(lam > 0, lam * lam * lam, 1.0), zero)

    lamc, nu = par["lam_c"], par["nu_c"]
    o = {"ext_c": torch.where(lamc > 0, (0.5 * math.pi) * NT_C * ((nu + 1) * (nu + 2)) / torch.where(lamc > 0, lamc * lamc, 1.0), zero),
         "ext_i": expo("i"), "ext_r": expo("r"), "ext_s": (0.5 * math.pi) * par["smob"], "ext_g": expo("g")}
    S = CFG["s_ratio"]
    o["ext"] = (((o["ext_c"] + o["ext_i"]) + o["ext_r"]) + o["ext_s"]) + o["ext_g"]
    o["bsc"] = (((o["ext_c"] / S[0] + o["ext_i"] / S[1]) + o["ext_r"] / S[2]) + o["ext_s"] / S[3]) + o["ext_g"] / S[4]
    o["bsc_mol"] = CFG["c_mol"] * (dev["p"] / (K_B * dev["t"]))
    em = (8.0 * math.pi / 3.0) * o["bsc_mol"]
    dt, dm = (CFG["eta"] * o["ext"] + em) * dz, em * dz
    below = lambda a: torch.cumsum(a, 1) - a                                      # noqa: E731
    above = lambda a: torch.flip(torch.cumsum(torch.flip(a, [1]), 1), [1]) - a     # noqa: E731
    E = lambda x: torch.where(x <= 700.0, torch.exp(-torch.clamp(x, max=700.0)), zero)   # noqa: E731
    g = lambda x: torch.where(x > 0, -torch.expm1(-x) / torch.where(x > 0, x, 1.0), 1.0)   # noqa: E731
    o["tau_up"], o["tau_dn"] = below(dt), above(dt)
    gl, gm = g(2.0 * dt), g(2.0 * dm)
    for d, tm in (("up", below(dm)), ("dn", above(dm))):
        o["att_" + d] = (o["bsc"] + o["bsc_mol"]) * E(2.0 * o["tau_" + d]) * gl
        o["sr_" + d] = o["att_" + d] / (o["bsc_mol"] * E(2.0 * tm) * gm)
    return o


def measure(a, ncol, lines):
    import numpy as np
    import torch
    import cases
    from kid_amd import LIDAR_INPUTS, LIDAR_NAMES, SPECTRA_PARAMS, SUMMARY_INPUTS, ThompsonMP

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # the state after one step
    ins = {k: dev[k] for k in LIDAR_INPUTS}
    sum_ins = {k: dev[k] for k in SUMMARY_INPUTS}
    dz = torch.from_numpy(np.full(NZ, 100.0)).to("cuda:0")
    variants = {
        "lidar_all": (lambda: m.lidar_profiles(ins, dz, CFG, LIDAR_NAMES, True), len(LIDAR_NAMES), 64),
        "lidar_att_up": (lambda: m.lidar_profiles(ins, dz, CFG, ("att_up",)), 1, 0),
        "lidar_ext": (lambda: m.lidar_profiles(ins, None, CFG, ("ext",)), 1, 0),
        "spectra_par": (lambda: m.size_spectra(ins, SPECTRA_PARAMS), len(SPECTRA_PARAMS), 0),
        "summary": (lambda: m.column_summary(sum_ins, dz), None, 0),
        "composite": (lambda: torch_composite(m, ins, dz), None, 0),
    }
    got, comp = m.lidar_profiles(ins, dz, CFG, LIDAR_NAMES), torch_composite(m, ins, dz)
    diff = {}
    for n in LIDAR_NAMES:
        ok = torch.isfinite(got[n]) & torch.isfinite(comp[n])
        diff[n] = float(((got[n] - comp[n]).abs()[ok] / got[n].abs()[ok].max().clamp(min=1e-300)).max())
    say("ncol=%-6d composite - lidar_all, max |difference| / max |profile|: %s" % (ncol, "  ".join("%s %.1e" % kv for kv in diff.items())))
    for _ in range(a.warmup):
        for fn, _n, _b in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, (fn, _n, _b) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"ncol": ncol, "nz": NZ, "reps": a.reps, "composite_max_diff": diff}
    base = statistics.median(times["spectra_par"])
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ratio_to_spectra_par": statistics.median(t) / base}
        nout, extra_bytes = variants[k][1], variants[k][2]
        extra = ""
        if nout is not None:
            res[k]["algo_bytes_per_column"] = (len(LIDAR_INPUTS) + nout) * NZ * 8 + extra_bytes
            res[k]["share_of_8TBs"] = res[k]["algo_bytes_per_column"] * ncol / (res[k]["ms_median"] * 1e-3) / HBM_PEAK
            extra = "   %6d B/column -> %5.1f %% of 8 TB/s" % (res[k]["algo_bytes_per_column"], 100.0 * res[k]["share_of_8TBs"])
        say("ncol=%-6d %-12s median %8.4f ms   min %8.4f   max %8.4f   x %6.3f of spectra_par%s"
            % (ncol, k, res[k]["ms_median"], min(t), max(t), res[k]["ratio_to_spectra_par"], extra))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_lidar.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_lidar: no GPU visible (this measurement has no CPU path)")
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_lidar.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0)),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = [measure(a, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "lidar_profiles", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
