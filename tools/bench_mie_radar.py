#!/usr/bin/env python
"""tools/bench_mie_radar.py -- time the cloud radar (kidmp_mie_radar_device, one launch of kidmp::k_mie_radar) on one MI355X
beside the reflectivity and the Doppler moments of the same state in the same context and a torch composite of the same
sums.

Workload, fp64, state in HBM, 10^5 and 10^4 columns x 120 levels: mixed-phase BASELINE config 3 after one column step (the
state of tools/bench_doppler.py) with dz = 100 m, a table at 3.19 mm on the scheme's own 100 bins per species.  All
variants run in ONE process, warmed up, taking turns launch by launch; every launch is timed with device events of its own
and the median of --reps (30) launches is reported with the minimum and maximum beside it.  Variants:
  mie_dbz        mie_radar, dbz alone
  mie_all        mie_radar, all fourteen outputs
  reflectivity   kidmp_reflectivity_device on the same state
  doppler        kidmp_doppler_moments_device, all nine outputs
  composite      mie_r, mie_s, mie_g, ext and dbz from torch operations on the device tensors: the load over [ncol, nz], the
                 five sums as [columns, nz, bins] tensors in chunks of columns (checked against mie_all once)
The share of levels that hold each species is printed.  Prints one line per variant and ONE JSON line at the end; the
lines also go to --out (profiles/r24_mie_radar.txt) under a header with the date."""
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
COL_CHUNK = 2048
# illustrative permittivities near 94 GHz (tests/test_gpu_mie_radar.py)
CFG = dict(wavelength=3.19e-3, eps_w=complex(7.7, 14.2), eps_i=complex(3.17, 0.01), rho_w=1000.0, rho_i=917.0, kw2=0.75)


def torch_load(c, d):
    """The load of tests/mie_radar_ref.py in torch on device tensors [ncol, nz] (tools/bench_radiometer.py shares it):
    (rho, species -> (present, ze, rho*q), density(x, D, dD) -> [ncol, nz, bins])."""
    import torch
    import doppler_ref as r
    import refl_oracle as ro
    t, p = d["t"], d["p"]
    qv = torch.clamp(d["qv"], min=1e-10)
    rho = 0.622 * p / (ro.R * t * (qv + 0.622))
    tiny = torch.full_like(t, 1.e-22)
    pr, ps, pg = d["qr"] > ro.R1, d["qs"] > ro.R2, d["qg"] > ro.R2
    rr = torch.where(pr, d["qr"] * rho, ro.R1)
    nr = torch.where(pr, torch.clamp(d["nr"] * rho, min=ro.R2), ro.R1)
    lamr = (ro.am_r * c["crg"][2] * c["org2"] * nr / rr) ** (1. / 3.)
    N0_r = nr * c["org2"] * lamr
    mvd_r = torch.where(pr, 3.672 / lamr, 50.E-6)
    ze_r = torch.where(pr, N0_r * c["crg"][3] / lamr ** 7, tiny)
    rs = torch.where(ps, d["qs"] * rho, ro.R1)
    tc0 = torch.clamp(t - 273.15, max=-0.1)
    fit = lambda a, x: (a[0] + a[1] * tc0 + a[2] * x + a[3] * tc0 * x + a[4] * tc0 * tc0 + a[5] * x * x + a[6] * tc0 * tc0 * x   # noqa: E731
                        + a[7] * tc0 * x * x + a[8] * tc0 * tc0 * tc0 + a[9] * x * x * x)
    smob = rs * c["oams"]
    moment = lambda x: 10.0 ** fit(ro.sa, x) * smob ** fit(ro.sb, x)   # noqa: E731
    ze_s = torch.where(ps, (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI) * (ro.am_s / 900.0) * (ro.am_s / 900.0) * moment(c["cse"][2]), tiny)
    rg = torch.where(pg, d["qg"] * rho, ro.R1)
    slw = (t < 270.65) & pr & (mvd_r > 100.E-6)
    xslw1 = torch.where(slw, 4.01 + torch.log10(mvd_r), 0.01)
    ygra1 = 4.31 + torch.log10(torch.clamp(rg, min=5.E-5))
    zans1 = 3.1 + (100. / (300. * xslw1 * ygra1 / (10. / xslw1 + 1. + 0.25 * ygra1) + 30. + 10. * ygra1))
    n0 = torch.clamp(10. ** zans1, min=ro.gonv_min, max=ro.gonv_max)
    n0 = torch.flip(torch.cummin(torch.flip(n0, [1]), 1).values, [1])
    lam_exp = (n0 * ro.am_g * c["cgg"][0] / rg) ** 0.25
    lamg = lam_exp * (c["cgg"][2] * c["ogg2"] * c["ogg1"]) ** c["obmg"]
    N0_g = n0 / (c["cgg"][1] * lam_exp) * lamg
    ze_g = torch.where(pg, (0.176 / 0.93) * (6.0 / ro.PI) * (6.0 / ro.PI) * (ro.am_g / 900.0) * (ro.am_g / 900.0)
                       * N0_g * c["cgg"][3] * (1. / lamg) ** 7, tiny)
    ratio = smob / moment(c["cse"][0])

    def density(x, D, dD):
        if x == "s":
            q = ratio[..., None]
            return (smob * ratio ** 3)[..., None] * (r.Kap0 * torch.exp(-q * r.Lam0 * D) + r.Kap1 * q ** r.mu_s * D ** r.mu_s * torch.exp(-q * r.Lam1 * D)) * dD
        N0, lam = (N0_r, lamr) if x == "r" else (N0_g, lamg)
        return N0[..., None] * torch.exp(-lam[..., None] * D) * dD

    return rho, {"r": (pr, ze_r, rr), "s": (ps, ze_s, rs), "g": (pg, ze_g, rg)}, density


def torch_composite(c, dev, table, kc, rho_w):
    """tests/mie_radar_ref.py in torch, on device tensors [ncol, nz]: mie_x, ext (no gas) and dbz."""
    import torch
    import refl_oracle as ro
    out = {n: torch.empty_like(dev["t"]) for n in ("mie_r", "mie_s", "mie_g", "ext", "dbz")}
    ncol = dev["t"].shape[0]
    for lo in range(0, ncol, COL_CHUNK):
        d = {k: v[lo:lo + COL_CHUNK] for k, v in dev.items()}
        rho, species, density = torch_load(c, d)
        ext = torch.zeros_like(rho)
        zp = {}
        for x, (has, ze, rq) in species.items():
            D, dD, rows = table[x]
            n = torch.where(has[..., None], density(x, D, dD), 0.0)
            A, B, E, M = ((n * rows[i]).sum(dim=2) for i in range(4))
            mie = torch.where(has & (B > 0), A / B, 1.0)
            ext = ext + torch.where(has & (M > 0), rq * E / M, 0.0)
            zp[x] = ze * mie
            out["mie_" + x][lo:lo + COL_CHUNK] = mie
        ext = torch.where(d["qc"] > ro.R1, ext + kc * (rho * d["qc"] / rho_w), ext)
        out["ext"][lo:lo + COL_CHUNK] = ext
        out["dbz"][lo:lo + COL_CHUNK] = 10. * torch.log10((zp["r"] + zp["s"] + zp["g"]) * 1.e18)
    return out


def measure(a, c, ncol, lines):
    import torch
    import cases
    import mie_radar_ref as ref
    from kid_amd import DOPPLER_NAMES, MIE_INPUTS, MIE_NAMES, MieCfg, ThompsonMP

    def say(s):
        print(s)
        lines.append(s)

    m = ThompsonMP(iiwarm=False, device=0)
    dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in cases.config3(ncol).items()}
    ppt = torch.zeros(ncol, 4, dtype=torch.float64, device="cuda:0")
    m.batch_step(dev, 10.0, ppt)                     # the state after one step
    ins = {k: dev[k] for k in MIE_INPUTS}
    dz = torch.full((NZ,), 100.0, dtype=torch.float64, device="cuda:0")
    table = m.mie_table(MieCfg(**CFG))
    rows = {x: tuple(torch.from_numpy(g).to("cuda:0") for g in table.get(x)) for x in ref.SPECIES}
    kc = ref.cloud_factor(ref.cfg_of(**CFG))
    variants = {
        "mie_dbz": lambda: m.mie_radar(table, ins, want=("dbz",)),
        "mie_all": lambda: m.mie_radar(table, ins, dz, want=MIE_NAMES),
        "reflectivity": lambda: m.reflectivity(ins),
        "doppler": lambda: m.doppler_moments(ins, want=DOPPLER_NAMES),
        "composite": lambda: torch_composite(c, ins, rows, kc, CFG["rho_w"]),
    }
    got, comp = variants["mie_all"](), variants["composite"]()
    share = {x: float((got["mie_" + x] != 1.0).sum().item()) / (ncol * NZ) for x in ref.SPECIES}
    diff = {n: float(((got[n] - comp[n]).abs() / (1.0 if n == "dbz" else comp[n].abs().clamp(min=1e-300))).max()) for n in comp}
    say("ncol=%-6d share of levels with mie_x != 1: %s" % (ncol, "  ".join("%s %.3f" % kv for kv in share.items())))
    say("ncol=%-6d composite - mie_all, max |difference| (dbz: dB; else relative): %s" % (ncol, "  ".join("%s %.1e" % kv for kv in diff.items())))
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
        say("ncol=%-6d %-12s median %9.4f ms   min %9.4f   max %9.4f" % (ncol, k, res[k]["ms_median"], min(t), max(t)))
    ms = {k: res[k]["ms_median"] for k in variants}
    res["ratios"] = {"mie_dbz/reflectivity": ms["mie_dbz"] / ms["reflectivity"], "mie_all/reflectivity": ms["mie_all"] / ms["reflectivity"],
                     "mie_all/doppler": ms["mie_all"] / ms["doppler"], "mie_all/mie_dbz": ms["mie_all"] / ms["mie_dbz"],
                     "mie_all/composite": ms["mie_all"] / ms["composite"]}
    # The exponentials of the densities (snow has two per bin) over the time of mie_dbz.  useful: those of the levels that
    # hold the species.  issued: an upper bound of what the kernel runs -- every lane of a level group walks the bin loop
    # when one of its levels holds the species, so all 120 levels count wherever the species occurs at all.
    per_bin = {x: len(rows[x][0]) * (2 if x == "s" else 1) for x in ref.SPECIES}
    res["useful_exp_per_s"] = ncol * NZ * sum(per_bin[x] * share[x] for x in ref.SPECIES) / (ms["mie_dbz"] * 1e-3)
    res["issued_exp_per_s_bound"] = ncol * NZ * sum(per_bin[x] for x in ref.SPECIES if share[x] > 0) / (ms["mie_dbz"] * 1e-3)
    say("ncol=%-6d ratios: %s" % (ncol, "  ".join("%s %.3f" % kv for kv in res["ratios"].items())))
    say("ncol=%-6d density exponentials per second in mie_dbz: useful (levels that hold the species) %.3e, issued at most "
        "(every lane of a live level group) %.3e" % (ncol, res["useful_exp_per_s"], res["issued_exp_per_s_bound"]))
    table.close()
    m.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ncols", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_mie_radar.txt"))
    a = ap.parse_args()
    import torch
    import doppler_ref as ref
    from oracle.oracle import Oracle
    if not torch.cuda.is_available():
        sys.exit("bench_mie_radar: no GPU visible (this measurement has no CPU path)")
    o = Oracle(iiwarm=True)
    c = ref.constants(o)
    o.close()
    lines = ["# tools/bench_mie_radar.py  %s  %s" % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0))]
    results = [measure(a, c, n, lines) for n in a.ncols]
    lines.append(json.dumps({"bench": "mie_radar", "device": torch.cuda.get_device_name(0), "results": results}))
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
