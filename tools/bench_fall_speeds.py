#!/usr/bin/env python
"""tools/bench_fall_speeds.py -- time the block-O fall speeds (kidmp_fall_speeds_device, one launch of kidmp::k_fall_speeds)
on one MI355X beside the other profile diagnostic of the same state and a torch composite of the same numbers.

Workloads: 10^5 and 10^4 mixed-phase columns x 120 levels (BASELINE config 3), fp64, after one column step, state in HBM.
All variants run in ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its
own and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  fall_all       all eleven profiles
  fall_total     flux_total alone
  fall_speeds    the six speeds alone
  dbz            kidmp_column_outputs_device, dbz alone, on the same state
  composite      the eleven profiles from torch operations on the device tensors (checked against fall_all once)
Algorithmic bytes per column of a fall_* variant: (9 profiles read + the requested ones written) * nz * 8; its share of
8 TB/s is printed.  Prints one line per variant and workload and ONE JSON line at the end; the lines also go
to --out (profiles/r13_fall_speeds.txt) under a header with the date and the library's fingerprint."""
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
SPEEDS = ("vt_r", "vt_nr", "vt_i", "vt_ni", "vt_s", "vt_g")


def torch_composite(c, dev):
    """tests/fall_speeds_ref.py in torch, on device tensors [ncol, nz]: the eleven profiles (default boost)."""
    import torch
    import fall_speeds_ref as r
    t, p = dev["t"], dev["p"]
    qv = torch.clamp(dev["qv"], min=1e-10)
    rho = 0.622 * p / (r.R * t * (qv + 0.622))
    rhof = torch.sqrt(r.RHO_NOT / rho)
    nz = t.shape[1]
    k = torch.arange(nz, device=t.device)[None, :]

    def inherit(own, has):
        src = torch.flip(torch.cummin(torch.flip(torch.where(has, k, nz), [1]), 1).values, [1])
        return torch.where(src < nz, own.gather(1, src.clamp(max=nz - 1)), torch.zeros_like(own))

    # load, M:1420-1492
    L = dev["qi"] > r.R1
    ri = torch.where(L, dev["qi"] * rho, r.R1)
    ni = torch.where(L, torch.clamp(dev["ni"] * rho, min=r.R2), r.R2)
    n_of = lambda lam: c["cig"][0] * c["oig2"] * ri / r.am_i * lam ** 3   # noqa: E731
    ni = torch.where(L & (ni <= r.R2), torch.clamp(n_of(c["cie"][1] / 25.E-6), max=499.E3), ni)
    xDi = 4.0 / (r.am_i * c["cig"][1] * c["oig1"] * ni / ri) ** (1. / 3.)
    ni = torch.where(L & (xDi < 5.E-6), torch.clamp(n_of(c["cie"][1] / 5.E-6), max=499.E3),
                     torch.where(L & (xDi > 300.E-6), n_of(c["cie"][1] / 300.E-6), ni))
    Lr = dev["qr"] > r.R1
    rr = torch.where(Lr, dev["qr"] * rho, r.R1)
    nr = torch.where(Lr, torch.clamp(dev["nr"] * rho, min=r.R2), r.R2)
    nr_of = lambda mvd: c["crg"][1] * c["org3"] * rr * (3.672 / mvd) ** 3 / r.am_r   # noqa: E731
    nr = torch.where(Lr & (nr <= r.R2), nr_of(1.0E-3), nr)
    mvd = 3.672 / (r.am_r * c["crg"][2] * c["org2"] * nr / rr) ** (1. / 3.)
    big, small = Lr & (mvd > 2.5E-3), Lr & (mvd < r.D0r * 0.75)
    mvd = torch.where(big, 2.5E-3, torch.where(small, r.D0r * 0.75, mvd))
    nr = torch.where(big, nr_of(2.5E-3), torch.where(small, nr_of(r.D0r * 0.75), nr))
    rs = torch.where(dev["qs"] > r.R1, dev["qs"] * rho, r.R1)
    rg = torch.where(dev["qg"] > r.R1, dev["qg"] * rho, r.R1)
    # rain and ice, M:3221-3269
    has_r, has_i, has_s, has_g = rr > r.R1, ri > r.R1, rs > r.R1, rg > r.R1
    lamr = (r.am_r * c["crg"][2] * c["org2"] * nr / rr) ** (1. / 3.)
    zero = torch.zeros_like(t)
    vtr = inherit(torch.where(has_r, rhof * r.av_r * c["crg"][5] * c["org3"] * lamr ** 4 / (lamr + r.fv_r) ** 5, zero), has_r)
    vtnr = inherit(torch.where(has_r, rhof * r.av_r * c["crg"][6] / c["crg"][11] * lamr ** 2.5 / (lamr + r.fv_r) ** 3.5, zero), has_r)
    ilami = 1. / (r.am_i * c["cig"][1] * c["oig1"] * ni / ri) ** (1. / 3.)
    vti = inherit(torch.where(has_i, rhof * r.av_i * c["cig"][2] * c["oig2"] * ilami, zero), has_i)
    vtni = inherit(torch.where(has_i, rhof * r.av_i * c["cig"][5] / c["cig"][6] * ilami, zero), has_i)
    # snow, block D and M:3288-3308
    tc0 = torch.clamp(t - 273.15, max=-0.1)
    x = c["cse"][0]
    fit = lambda a: (a[0] + a[1] * tc0 + a[2] * x + a[3] * tc0 * x + a[4] * tc0 * tc0 + a[5] * x * x + a[6] * tc0 * tc0 * x   # noqa: E731
                     + a[7] * tc0 * x * x + a[8] * tc0 * tc0 * tc0 + a[9] * x * x * x)
    smob = rs * c["oams"]
    smoc = 10.0 ** fit(r.sa) * smob ** fit(r.sb)
    Mrat = smob / smoc
    mm = Mrat ** r.mu_s
    t12 = r.Kap0 * c["csg"][3] / (Mrat * r.Lam0 + r.fv_s) ** c["cse"][3] + r.Kap1 * mm * c["csg"][9] / (Mrat * r.Lam1 + r.fv_s) ** c["cse"][9]
    t34 = r.Kap0 * c["csg"][0] / (Mrat * r.Lam0) ** 3 + r.Kap1 * mm * c["csg"][6] / (Mrat * r.Lam1) ** c["cse"][6]
    vts = rhof * r.av_s * t12 / t34
    boost = torch.where(t < r.T_0, 1.0, 1.5)
    own = torch.where(t > r.T_0 + 0.1, torch.maximum(vts * boost, vts * ((vtr - vts * boost) / (t - r.T_0))), vts * boost)
    vtsk = inherit(torch.where(has_s, own, zero), has_s)
    # graupel, block E and M:3325-3334
    k_0 = torch.where(t >= 270.65, k, 0).max(1, keepdim=True).values
    slw = (k > k_0) & Lr & (mvd > 100.E-6)
    xslw1 = torch.where(slw, 4.01 + torch.log10(mvd), 0.01)
    ygra1 = 4.31 + torch.log10(torch.clamp(rg, min=5.E-5))
    zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1))
    n0 = torch.clamp(10. ** zans1, min=r.gonv_min, max=r.gonv_max)
    n0 = torch.flip(torch.cummin(torch.flip(n0, [1]), 1).values, [1])
    lamg = (n0 * r.am_g * c["cgg"][0] / rg) ** 0.25 * (c["cgg"][2] * c["ogg2"] * c["ogg1"]) ** c["obmg"]
    vtg = rhof * r.av_g * c["cgg"][5] * c["ogg3"] * (1. / lamg) ** r.bv_g
    vtgk = inherit(torch.where(has_g, torch.where(t > r.T_0, torch.maximum(vtg, vtr), vtg), zero), has_g)
    out = dict(vt_r=vtr, vt_nr=vtnr, vt_i=vti, vt_ni=vtni, vt_s=vtsk, vt_g=vtgk,
               flux_r=vtr * rr, flux_i=vti * ri, flux_s=vtsk * rs, flux_g=vtgk * rg)
    out["flux_total"] = ((out["flux_r"] + out["flux_i"]) + out["flux_s"]) + out["flux_g"]
    return out


def measure(a, c, ncol, lines):
    import torch
    import cases
    from kid_amd import FALL_INPUTS, FALL_NAMES, ThompsonMP

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # the state after one step
    ins = {k: dev[k] for k in FALL_INPUTS}
    variants = {
        "fall_all": (lambda: m.fall_speeds(ins), len(FALL_NAMES)),
        "fall_total": (lambda: m.fall_speeds(ins, want=("flux_total",)), 1),
        "fall_speeds": (lambda: m.fall_speeds(ins, want=SPEEDS), len(SPEEDS)),
        "dbz": (lambda: m.column_outputs(dev, dbz=True, radii=False), None),
        "composite": (lambda: torch_composite(c, ins), None),
    }
    got, comp = m.fall_speeds(ins), torch_composite(c, ins)
    # relative to the profile's own maximum: the snow speed above T_0 + 0.1 is a difference (M:3301-3302)
    diff = {n: float((got[n] - comp[n]).abs().max() / got[n].abs().max().clamp(min=1e-300)) for n in FALL_NAMES}
    rel = max(diff.values())
    say("ncol=%-6d composite - fall_all, max |difference| / max |profile|: %s" % (ncol, "  ".join("%s %.1e" % (n, d) for n, d in diff.items())))
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
    res = {"ncol": ncol, "nz": NZ, "reps": a.reps, "composite_max_diff_over_max": diff}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        nout = variants[k][1]
        extra = ""
        if nout is not None:
            res[k]["algo_bytes_per_column"] = (len(FALL_INPUTS) + nout) * NZ * 8
            res[k]["share_of_8TBs"] = res[k]["algo_bytes_per_column"] * ncol / (res[k]["ms_median"] * 1e-3) / HBM_PEAK
            extra = "   %6d B/column -> %5.1f %% of 8 TB/s" % (res[k]["algo_bytes_per_column"], 100.0 * res[k]["share_of_8TBs"])
        say("ncol=%-6d %-12s median %8.4f ms   min %8.4f   max %8.4f%s" % (ncol, k, res[k]["ms_median"], min(t), max(t), extra))
    ms = {k: res[k]["ms_median"] for k in variants}
    say("ncol=%-6d fall_all %.2fx composite; fall_total %.2fx dbz; composite agrees to %.1e of each profile's maximum"
        % (ncol, ms["fall_all"] / ms["composite"], ms["fall_total"] / ms["dbz"], rel))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_fall_speeds.txt"))
    a = ap.parse_args()
    import torch
    import fall_speeds_ref as ref
    import kid_amd
    from oracle.oracle import Oracle
    if not torch.cuda.is_available():
        sys.exit("bench_fall_speeds: no GPU visible (this measurement has no CPU path)")
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_fall_speeds.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0)),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = [measure(a, c, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "fall_speeds", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
