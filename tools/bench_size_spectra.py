#!/usr/bin/env python
"""tools/bench_size_spectra.py -- time the size spectra (kidmp_size_spectra_device, one launch of kidmp::k_size_spectra) on
one MI355X beside a torch composite that forms the same bins from the kernel's own parameters, and beside the store roofline.

Workloads: 10^4 and 10^3 mixed-phase columns x 120 levels (BASELINE config 3), fp64, after one column step, state in HBM,
the scheme's own 100 bins per species (all five species at 10^5 columns would be 48 GB).  All variants run in ONE process,
warmed up, taking turns launch by launch, into tensors allocated beforehand; every launch is timed with device events of
its own and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  params          the eleven parameter profiles alone
  rain            N_r alone
  all5            the five spectra
  composite_rain  N_r from torch operations on lam_r, n0_r and the grid (checked against `rain` once)
  composite_all5  the five spectra from torch operations on the eleven parameters (checked against `all5` once)
Store roofline of a spectrum: nb * nz * 8 B per species and column at 8 TB/s; the share of it is printed.  Prints one line
per variant and workload and ONE JSON line at the end; the lines also go to --out (profiles/r17_size_spectra.txt) under a
header with the date and the library's fingerprint."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NZ, NB = 120, 100
HBM_PEAK = 8.0e12


def torch_composite(par, grids, species):
    """The bins of `species` from the parameter profiles [ncol, nz] and the grids (D, dD) [nb]: the formulas of
    include/kidmp_spectra.h with the 700 rule, [ncol, nb, nz] each."""
    import torch
    import size_spectra_ref as r

    def e(k):
        return par[k][:, None, :]

    def exp_neg(x):
        return torch.where(x <= r.EXP_MAX, torch.exp(-torch.clamp(x, max=r.EXP_MAX)), torch.zeros_like(x))

    out = {}
    for x in species:
        D, dD = grids[x][0][None, :, None], grids[x][1][None, :, None]
        if x in ("r", "i", "g"):
            out[x] = e("n0_" + x) * exp_neg(e("lam_" + x) * D) * dD
        elif x == "c":
            out[x] = e("n0_c") * D ** e("nu_c") * exp_neg(e("lam_c") * D) * dD
        else:
            has = e("smob") > 0
            ratio = torch.where(has, e("smob") / torch.where(has, e("smoc"), torch.ones_like(e("smoc"))), torch.ones_like(e("smob")))
            n = e("smob") * ratio ** 3 * (r.Kap0 * exp_neg(ratio * r.Lam0 * D) + r.Kap1 * ratio ** r.mu_s * D ** r.mu_s * exp_neg(ratio * r.Lam1 * D)) * dD
            out[x] = torch.where(has, n, torch.zeros_like(n))
    return out


def measure(a, ncol, lines):
    import torch
    import cases
    from kid_amd import SPECTRA_INPUTS, SPECTRA_PARAMS, SPECTRA_SPECIES, ThompsonMP, default_grid

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                 # the state after one step
    ins = {k: dev[k] for k in SPECTRA_INPUTS}
    grids = {x: tuple(torch.from_numpy(g).to("cuda:0") for g in default_grid(m, x)) for x in SPECTRA_SPECIES}
    out = {n: torch.empty((ncol, NZ), dtype=torch.float64, device="cuda:0") for n in SPECTRA_PARAMS}
    out.update({x: torch.empty((ncol, NB, NZ), dtype=torch.float64, device="cuda:0") for x in SPECTRA_SPECIES})
    par = m.size_spectra(ins, SPECTRA_PARAMS)
    variants = {
        "params": (lambda: m.size_spectra(ins, SPECTRA_PARAMS, out=out), 0),
        "rain": (lambda: m.size_spectra(ins, ("r",), out=out), 1),
        "all5": (lambda: m.size_spectra(ins, SPECTRA_SPECIES, out=out), 5),
        "composite_rain": (lambda: torch_composite(par, grids, ("r",)), 1),
        "composite_all5": (lambda: torch_composite(par, grids, SPECTRA_SPECIES), 5),
    }
    got, comp = m.size_spectra(ins, SPECTRA_SPECIES), torch_composite(par, grids, SPECTRA_SPECIES)
    # relative to the spectrum's own maximum
    diff = {x: float((got[x] - comp[x]).abs().max() / got[x].abs().max().clamp(min=1e-300)) for x in SPECTRA_SPECIES}
    say("ncol=%-6d composite - all5, max |difference| / max |spectrum|: %s" % (ncol, "  ".join("%s %.1e" % (x, d) for x, d in diff.items())))
    del got, comp
    for _ in range(a.warmup):
        for fn, _n in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, (fn, _n) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
            del r
    res = {"ncol": ncol, "nz": NZ, "nb": NB, "reps": a.reps, "composite_max_diff_over_max": diff}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        nspec = variants[k][1]
        extra = ""
        if nspec:
            res[k]["store_bytes_per_column"] = nspec * NB * NZ * 8
            res[k]["roofline_ms"] = res[k]["store_bytes_per_column"] * ncol / HBM_PEAK * 1e3
            res[k]["share_of_8TBs"] = res[k]["roofline_ms"] / res[k]["ms_median"]
            extra = "   %7d B/column stored -> roofline %7.4f ms, %5.1f %% of 8 TB/s" % (res[k]["store_bytes_per_column"], res[k]["roofline_ms"],
                                                                                       100.0 * res[k]["share_of_8TBs"])
        say("ncol=%-6d %-15s median %9.4f ms   min %9.4f   max %9.4f%s" % (ncol, k, res[k]["ms_median"], min(t), max(t), extra))
    ms = {k: res[k]["ms_median"] for k in variants}
    say("ncol=%-6d rain %.3fx composite_rain; all5 %.3fx composite_all5; composite agrees to %.1e of each spectrum's maximum"
        % (ncol, ms["rain"] / ms["composite_rain"], ms["all5"] / ms["composite_all5"], max(diff.values())))
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ncols", type=int, nargs="+", default=[10000, 1000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_size_spectra.txt"))
    a = ap.parse_args()
    import torch
    import kid_amd
    if not torch.cuda.is_available():
        sys.exit("bench_size_spectra: no GPU visible (this measurement has no CPU path)")
    m = kid_amd.ThompsonMP(iiwarm=True, device=0)
    lines = ["# tools/bench_size_spectra.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0)),
             "# fingerprint: %s" % m.kernel_fingerprint()]
    m.close()
    results = [measure(a, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "size_spectra", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
