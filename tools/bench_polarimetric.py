#!/usr/bin/env python
"""tools/bench_polarimetric.py -- time the polarimetric radar (kidmp_polarimetric_device, one launch of
kidmp::k_polarimetric) on one MI355X beside the reflectivity and the cloud radar's dbz of the same state in the same
context and a torch composite of the same sums.

Workload, fp64, state in HBM, 10^5 and 10^4 columns x 120 levels: mixed-phase BASELINE config 3 after one column step (the
state of tools/bench_mie_radar.py), tables at 10 cm on the scheme's own 100 bins per species.  All variants run in ONE
process, warmed up, taking turns launch by launch; every launch is timed with device events of its own and the median of
--reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  pol_all         polarimetric, all thirteen outputs, the default table (graupel uniform: no bins, no density)
  pol_zdr         zdr alone
  pol_kdp_r       kdp_r alone (rain's bins only)
  pol_all_quad    all thirteen outputs, force_quadrature = 1 (graupel walks its bins too)
  pol_zdr_quad    zdr alone, force_quadrature = 1
  reflectivity    kidmp_reflectivity_device on the same state
  mie_dbz         kidmp_mie_radar_device, dbz alone, the default 10-cm Mie table on the same bins
  composite       dbz_h, zdr, kdp and rhohv from torch operations on the device tensors: the load over [ncol, nz], the seven
                  sums as [columns, nz, bins] tensors in chunks of columns, graupel by its bins (checked against
                  pol_all_quad once)
The share of levels that hold each species is printed.  Prints one line per variant and ONE JSON line at the end; the
lines also go to --out (profiles/r26_polarimetric.txt) under a header with the date."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

NZ = 120
COL_CHUNK = 2048


def torch_composite(c, dev, table, kfac):
    """tests/polarimetric_ref.py in torch, on device tensors [ncol, nz], every species by its bins: dbz_h, zdr, kdp, rhohv."""
    import torch
    from bench_mie_radar import torch_load
    out = {n: torch.empty_like(dev["t"]) for n in ("dbz_h", "zdr", "kdp", "rhohv")}
    ncol = dev["t"].shape[0]
    for lo in range(0, ncol, COL_CHUNK):
        d = {k: v[lo:lo + COL_CHUNK] for k, v in dev.items()}
        rho, species, density = torch_load(c, d)
        Zh, Zv, Cr, Ci, Kd = (torch.zeros_like(rho) for _ in range(5))
        for x, (has, ze, rq) in species.items():
            D, dD, rows = table[x]
            n = torch.where(has[..., None], density(x, D, dD), 0.0)
            H, V, Xr, Xi, S, K, M = ((n * rows[i]).sum(dim=2) for i in range(7))
            ok = has & (S > 0)
            Ss = torch.where(ok, S, 1.0)
            Zh = Zh + ze * torch.where(ok, H / Ss, 1.0)
            Zv = Zv + ze * torch.where(ok, V / Ss, 1.0)
            Cr = Cr + ze * torch.where(ok, Xr / Ss, 1.0)
            Ci = Ci + ze * torch.where(ok, Xi / Ss, 0.0)
            okm = has & (M > 0)
            rqx = d["qr"] * rho if x == "r" else rq
            Kd = Kd + torch.where(okm, (kfac * rqx) * (K / torch.where(okm, M, 1.0)), 0.0)
        sl = slice(lo, lo + COL_CHUNK)
        out["dbz_h"][sl] = 10. * torch.log10(Zh * 1.e18)
        out["zdr"][sl] = 10. * torch.log10(Zh / Zv)
        out["kdp"][sl] = Kd
        out["rhohv"][sl] = torch.clamp(torch.sqrt(Cr * Cr + Ci * Ci) / torch.sqrt(Zh * Zv), max=1.0)
    return out


def measure(a, c, ncol, lines):
    import torch
    import cases
    import polarimetric_ref as ref
    from kid_amd import POL_INPUTS, POL_NAMES, PolCfg, ThompsonMP

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                     # the state after one step
    ins = {k: dev[k] for k in POL_INPUTS}
    mie_ins = dict(ins, qc=dev["qc"])
    table, quad, mie = m.pol_table(), m.pol_table(None, PolCfg(force_quadrature=True)), m.mie_table()
    assert table.get("g")[3] and not quad.get("g")[3]
    rows = {x: tuple(torch.from_numpy(g).to("cuda:0") for g in quad.get(x)[:3]) for x in ref.SPECIES}
    kfac = ref.kfac(0.10)
    variants = {
        "pol_all": lambda: m.polarimetric(table, ins, want=POL_NAMES),
        "pol_zdr": lambda: m.polarimetric(table, ins, want=("zdr",)),
        "pol_kdp_r": lambda: m.polarimetric(table, ins, want=("kdp_r",)),
        "pol_all_quad": lambda: m.polarimetric(quad, ins, want=POL_NAMES),
        "pol_zdr_quad": lambda: m.polarimetric(quad, ins, want=("zdr",)),
        "reflectivity": lambda: m.reflectivity(ins),
        "mie_dbz": lambda: m.mie_radar(mie, mie_ins, want=("dbz",)),
        "composite": lambda: torch_composite(c, ins, rows, kfac),
    }
    got, comp = variants["pol_all_quad"](), variants["composite"]()
    share = {x: float((got["kdp_" + x] != 0.0).sum().item()) / (ncol * NZ) for x in ref.SPECIES}
    lin = math.log(10.0) / 10.0
    diff = {"dbz_h": float((got["dbz_h"] - comp["dbz_h"]).abs().max()) * lin, "zdr": float((got["zdr"] - comp["zdr"]).abs().max()) * lin,
            "kdp": float(((got["kdp"] - comp["kdp"]).abs() / comp["kdp"].abs().clamp(min=1e-300)).max()),
            "rhohv": float((got["rhohv"] - comp["rhohv"]).abs().max())}
    say("ncol=%-6d share of levels with kdp_x != 0: %s" % (ncol, "  ".join("%s %.3f" % kv for kv in share.items())))
    say("ncol=%-6d composite - pol_all_quad, max |difference| (dbz_h, zdr: of the linear quantity; kdp relative; rhohv absolute): %s"
        % (ncol, "  ".join("%s %.1e" % kv for kv in diff.items())))
    say("ncol=%-6d largest zdr %.3f dB, kdp %.3f deg/km, smallest rhohv %.5f"
        % (ncol, float(got["zdr"].max()), float(got["kdp"].max()), float(got["rhohv"].min())))
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    res = {"ncol": ncol, "nz": NZ, "reps": a.reps, "share": share, "composite_max_diff": diff}
    for k, t in times.items():
        res[k] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t)}
        say("ncol=%-6d %-13s median %9.4f ms   min %9.4f   max %9.4f" % (ncol, k, res[k]["ms_median"], min(t), max(t)))
    ms = {k: res[k]["ms_median"] for k in variants}
    res["ratios"] = {"pol_all/mie_dbz": ms["pol_all"] / ms["mie_dbz"], "pol_zdr/mie_dbz": ms["pol_zdr"] / ms["mie_dbz"],
                     "pol_all_quad/mie_dbz": ms["pol_all_quad"] / ms["mie_dbz"], "pol_all/pol_all_quad": ms["pol_all"] / ms["pol_all_quad"],
                     "pol_zdr/pol_zdr_quad": ms["pol_zdr"] / ms["pol_zdr_quad"], "pol_kdp_r/pol_zdr": ms["pol_kdp_r"] / ms["pol_zdr"],
                     "pol_all/reflectivity": ms["pol_all"] / ms["reflectivity"], "pol_all_quad/composite": ms["pol_all_quad"] / ms["composite"]}
    say("ncol=%-6d ratios: %s" % (ncol, "  ".join("%s %.3f" % kv for kv in res["ratios"].items())))
    for t in (table, quad, mie):
        t.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_polarimetric.txt"))
    a = ap.parse_args()
    import torch
    import doppler_ref as ref
    from oracle.oracle import Oracle
    if not torch.cuda.is_available():
        sys.exit("bench_polarimetric: no GPU visible (this measurement has no CPU path)")
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    lines = ["# tools/bench_polarimetric.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0))]
    results = [measure(a, c, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "polarimetric", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
